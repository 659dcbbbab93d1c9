"""TEST INFRASTRUCTURE: the stereo depth of DESIGN.md section 4, "Stereo depth" (csrc/gf_stereo_depth.hpp), restated in numpy float64 operation for operation,
with the lifts of PINHOLE, MEI, PINHOLE_FULL and SCARAMUZZA (csrc/gf_camera_models.hpp) and of a KANNALA_BRANDT camera without distortion coefficients
(theta == r; its sin / cos / atan2 are numpy's, so that model is held to a count, not to the bit).  Also the cases the stereo-depth tests share.  A camera here
is a dict(model, proj, dist, xi, poly, affine); gf(cam) is its gfamd.CameraModelEx."""
import numpy as np

WHY = {"no_match": 1, "lift": 2, "parallax": 3, "behind": 4, "epipolar": 5, "range": 6, "ok": 7}   # GF_STEREO_DEPTH_*
NAMES = {v: k for k, v in WHY.items()}
MODEL_ID = {"PINHOLE": 0, "MEI": 1, "KANNALA_BRANDT": 2, "PINHOLE_FULL": 3, "SCARAMUZZA": 4}
F8 = np.float64


def camera(model, proj=(0, 0, 0, 0), dist=(), xi=0.0, poly=(), affine=()):
    pad = lambda v, n: tuple(float(x) for x in v) + (0.0,) * (n - len(v))
    return dict(model=model, proj=pad(proj, 4), dist=pad(dist, 8), xi=float(xi), poly=pad(poly, 5), affine=pad(affine, 5))


def gf(cam):
    import gfamd
    return gfamd.CameraModelEx.make(cam["model"], cam["proj"], cam["dist"], cam["xi"], cam["poly"], (), cam["affine"])


def cfg(R, t, max_depth, min_depth=0.1, min_parallax=1e-3, max_epipolar=10.0 / 460.0, right_obs=1, enable=1):
    return dict(enable=enable, right_obs=right_obs, R=tuple(float(v) for v in np.asarray(R, F8).reshape(9)), t=tuple(float(v) for v in t),
                min_parallax=float(min_parallax), max_epipolar=float(max_epipolar), min_depth=float(min_depth), max_depth=float(max_depth))


def gf_cfg(c):
    import gfamd
    return gfamd.StereoDepthCfg.make(c["R"], c["t"], c["max_depth"], c["min_depth"], c["min_parallax"], c["max_epipolar"], c["right_obs"], c["enable"])


def rot(rx, ry, rz):
    """Rz Ry Rx, row-major tuple of 9"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return tuple(float(v) for v in (Rz @ Ry @ Rx).reshape(9))


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


# ---- the lifts (gfcam::lift), every operation in the order the header writes it
def _distortion(k1, k2, p1, p2, x, y):
    mx2, my2, mxy = x * x, y * y, x * y
    rho2 = mx2 + my2
    rad = k1 * rho2 + k2 * rho2 * rho2
    return x * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2), y * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)


def _undistort(proj, dist, u, v):
    fx, fy, cx, cy = [F8(x) for x in proj]
    k1, k2, p1, p2 = [F8(x) for x in dist[:4]]
    i11, i13, i22, i23 = 1.0 / fx, -cx / fx, 1.0 / fy, -cy / fy
    mx_d, my_d = i11 * u + i13, i22 * v + i23
    if k1 == 0 and k2 == 0 and p1 == 0 and p2 == 0:
        return mx_d, my_d
    dx, dy = _distortion(k1, k2, p1, p2, mx_d, my_d)
    X, Y = mx_d - dx, my_d - dy
    for _ in range(7):
        dx, dy = _distortion(k1, k2, p1, p2, X, Y)
        X, Y = mx_d - dx, my_d - dy
    return X, Y


def lift(cam, uv):
    """[n, 2] float32 pixels -> [n, 3] float64 rays, as gfcam::lift"""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    u, v = uv[:, 0].astype(F8), uv[:, 1].astype(F8)
    m = cam["model"]
    with np.errstate(all="ignore"):
        if m == "PINHOLE":
            X, Y = _undistort(cam["proj"], cam["dist"], u, v)
            return np.stack([X, Y, np.ones_like(X)], 1)
        if m == "MEI":
            X, Y = _undistort(cam["proj"], cam["dist"], u, v)
            xi = F8(cam["xi"])
            if xi == 1.0:
                Z = (1.0 - X * X - Y * Y) / 2.0
            else:
                rho2 = X * X + Y * Y
                Z = 1.0 - xi * (rho2 + 1.0) / (xi + np.sqrt(1.0 + (1.0 - xi * xi) * rho2))
            return np.stack([X, Y, Z], 1)
        if m == "PINHOLE_FULL":
            fx, fy, cx, cy = [F8(x) for x in cam["proj"]]
            k1, k2, p1, p2, k3, k4, k5, k6 = [F8(x) for x in cam["dist"]]
            ifx, ify, i13, i23 = 1. / fx, 1. / fy, -cx / fx, -cy / fy
            x0, y0 = ifx * u + i13, ify * v + i23
            x, y = x0, y0
            for _ in range(9):
                r2 = x * x + y * y
                icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
                deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
                deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
                x, y = (x0 - deltaX) * icdist, (y0 - deltaY) * icdist
            return np.stack([x, y, np.ones_like(x)], 1)
        if m == "SCARAMUZZA":
            p = [F8(x) for x in cam["poly"]]
            ac, ad, ae, ccx, ccy = [F8(x) for x in cam["affine"]]
            inv_scale = 1.0 / (ac - ad * ae)
            xc0, xc1 = u - ccx, v - ccy
            xa0, xa1 = inv_scale * (xc0 - ad * xc1), inv_scale * (-ae * xc0 + ac * xc1)
            phi = np.sqrt(xa0 * xa0 + xa1 * xa1)
            phi_i, z = np.ones_like(phi), np.zeros_like(phi)
            for i in range(5):
                z = z + phi_i * p[i]
                phi_i = phi_i * phi
            return np.stack([xc0, xc1, -z], 1)
        if m == "KANNALA_BRANDT":
            assert all(x == 0 for x in cam["dist"]), "the restatement covers the camera without distortion coefficients (theta == r)"
            mu, mv, u0, v0 = [F8(x) for x in cam["proj"]]
            px, py = (1.0 / mu) * u + (-u0 / mu), (1.0 / mv) * v + (-v0 / mv)
            rho = np.sqrt(px * px + py * py)
            phi = np.where(rho < 1e-10, 0.0, np.arctan2(py, px))
            st = np.sin(rho)
            return np.stack([st * np.cos(phi), st * np.sin(phi), np.cos(rho)], 1)
    raise ValueError(m)


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def parts(left, right, c, lu, ru):
    """every intermediate of the definition, per point, whatever the gates say (dict of [n] float64)"""
    with np.errstate(all="ignore"):
        Pl, Pr = lift(left, lu), lift(right, ru)
        R, t = [F8(v) for v in c["R"]], [F8(v) for v in c["t"]]
        a = [Pl[:, 0] / Pl[:, 2], Pl[:, 1] / Pl[:, 2], np.ones(len(Pl))]
        bx, by = Pr[:, 0] / Pr[:, 2], Pr[:, 1] / Pr[:, 2]
        d = [(R[0] * bx + R[1] * by) + R[2], (R[3] * bx + R[4] * by) + R[5], (R[6] * bx + R[7] * by) + R[8]]
        aa, dd, ad, at, dt = _dot(a, a), _dot(d, d), _dot(a, d), _dot(a, t), _dot(d, t)
        den = aa * dd - ad * ad
        s, u = (at * dd - ad * dt) / den, (at * ad - aa * dt) / den
        w = [s * a[0] - t[0], s * a[1] - t[1], s * a[2] - t[2]]
        qx, qy, qz = (R[0] * w[0] + R[3] * w[1]) + R[6] * w[2], (R[1] * w[0] + R[4] * w[1]) + R[7] * w[2], (R[2] * w[0] + R[5] * w[1]) + R[8] * w[2]
        ex, ey = qx - bx * qz, qy - by * qz
        return dict(Pl=Pl, Pr=Pr, aa=aa, dd=dd, den=den, s=s, u=u, qz=qz, e2=ex * ex + ey * ey, m=np.rint(1000.0 * s))


def depth(left, right, c, lu, ru, status):
    """gfsd::depth_of on every point -> (depth_mm uint16, why uint8)"""
    lu, ru = np.asarray(lu, np.float32).reshape(-1, 2), np.asarray(ru, np.float32).reshape(-1, 2)
    status = np.asarray(status, np.uint8).reshape(-1)
    n = len(lu)
    p = parts(left, right, c, lu, ru)
    par2, epi2 = F8(c["min_parallax"]) * F8(c["min_parallax"]), F8(c["max_epipolar"]) * F8(c["max_epipolar"])
    lo = 1000.0 * F8(c["min_depth"])
    hi = 1000.0 * F8(c["max_depth"]) if 1000.0 * F8(c["max_depth"]) < 65535.0 else F8(65535.0)
    with np.errstate(all="ignore"):
        gates = [(WHY["no_match"], status == 0),
                 (WHY["lift"], ~(np.isfinite(p["Pl"]).all(1) & np.isfinite(p["Pr"]).all(1)) | (p["Pl"][:, 2] <= 0.0) | (p["Pr"][:, 2] <= 0.0)),
                 (WHY["parallax"], p["den"] <= (par2 * p["aa"]) * p["dd"]),
                 (WHY["behind"], (p["s"] <= 0.0) | (p["u"] <= 0.0)),
                 (WHY["epipolar"], (p["qz"] <= 0.0) | (p["e2"] > epi2 * (p["qz"] * p["qz"]))),
                 (WHY["range"], ~((p["m"] >= lo) & (p["m"] <= hi)))]
    why = np.full(n, WHY["ok"], np.uint8)
    for code, fires in reversed(gates):   # the first gate that fires names the reason
        why[fires] = code
    mm = np.zeros(n, np.uint16)
    ok = why == WHY["ok"]
    mm[ok] = p["m"][ok].astype(np.uint16)
    return mm, why


def census(why):
    return {k: int((np.asarray(why) == v).sum()) for k, v in WHY.items()}


# ---- cameras and rigs the tests share
PIN = camera("PINHOLE", (400.0, 401.0, 160.0, 120.5), (0.148, -0.468, 0.0016, -0.0089))                  # distorted (the coefficients of config/realsense/idc_cam.yaml)
PIN_PLAIN = camera("PINHOLE", (400.0, 400.0, 160.0, 120.0))
FULL = camera("PINHOLE_FULL", (398.0, 399.0, 161.0, 119.0), (0.12, -0.2, 0.0007, -0.0011, 0.05, 0.02, -0.01, 0.003))
MEI = camera("MEI", (300.0, 301.0, 158.0, 121.0), (-0.05, 0.01, 0.0003, -0.0002), xi=1.2)
MEI1 = camera("MEI", (300.0, 300.0, 160.0, 120.0), xi=1.0)                                                # the xi == 1 branch; P.z <= 0 from 300 px off the centre
SCA = camera("SCARAMUZZA", poly=(-400.0, 0.0, 0.0011, -1.0e-7, 2.0e-10), affine=(1.0005, 0.0002, -0.0001, 160.3, 119.6))
KB = camera("KANNALA_BRANDT", (400.0, 400.0, 160.0, 120.0))
RECT = dict(R=IDENTITY, t=(0.05, 0.0, 0.0))                                 # the right eye 0.05 m to the right of the left: p_left = p_right + t
TILT = dict(R=rot(0.01, -0.015, 0.02), t=(0.11, -0.03, 0.004))              # a rotated, vertically offset right eye


def project(cam, xyz):
    """spaceToPlane on the host through the library (gfamd.camera_project) -> [n, 2] float64"""
    import gfamd
    return gfamd.camera_project([gf(cam)], [np.asarray(xyz, F8).reshape(-1, 3)])[0]


def planted(left, right, rig, n, seed, z_lo=0.5, z_hi=8.0, spread=0.25):
    """n points in front of the left camera with z at millimetre centres plus 0.25 mm, and their pixels in both eyes by the host projection, as float32"""
    g = np.random.default_rng(seed)
    z = np.floor(g.uniform(z_lo, z_hi, n) * 1000.0) / 1000.0 + 0.00025
    xyz = np.stack([g.uniform(-spread, spread, n) * z, g.uniform(-spread, spread, n) * z, z], 1)
    R, t = np.asarray(rig["R"], F8).reshape(3, 3), np.asarray(rig["t"], F8)
    right_xyz = (xyz - t) @ R          # R^T (p - t), row by row
    return xyz, project(left, xyz).astype(np.float32), project(right, right_xyz).astype(np.float32)


# ---- the cases.  One case is one set of the building block: dict(name, left, right, cfg, lu, ru, st)
def plant_from_left(left, right, rig, lu, z):
    """the right pixels of the points at depth z (along the left z axis) on the rays of the left pixels lu: the left ray by the restatement's lift, the right pixel
    by the host projection -> float32 [n, 2]"""
    lu = np.asarray(lu, np.float32).reshape(-1, 2)
    P = lift(left, lu)
    xyz = np.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], np.ones(len(P))], 1) * np.asarray(z, F8).reshape(-1, 1)
    R, t = np.asarray(rig["R"], F8).reshape(3, 3), np.asarray(rig["t"], F8)
    return project(right, (xyz - t) @ R).astype(np.float32)


def _case(name, left, right, c, lu, ru, st=None):
    lu, ru = np.ascontiguousarray(lu, np.float32).reshape(-1, 2), np.ascontiguousarray(ru, np.float32).reshape(-1, 2)
    st = np.ones(len(lu), np.uint8) if st is None else np.ascontiguousarray(st, np.uint8)
    return dict(name=name, left=left, right=right, cfg=c, lu=lu, ru=ru, st=st)


def _flip(pred, lo, hi):
    """neighbouring doubles (a, b), a < b, with pred(a) != pred(b), between lo and hi where pred differs"""
    plo = pred(lo)
    assert plo != pred(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            return lo, hi
        if pred(mid) == plo:
            lo = mid
        else:
            hi = mid


def _grid(n, seed, w=320, h=240, margin=40):
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(margin, w - margin, n), g.uniform(margin, h - margin, n)], 1).astype(np.float32)


TIE_CAM = camera("PINHOLE", (512.0, 512.0, 160.0, 120.0))   # powers of two: the centre pixel lifts to (0, 0, 1) and pixel (144, 120) to (-2^-5, 0, 1) exactly


def tie_cases():
    """(case, expected counts): a rectified rig in which s == 32 t.x exactly, its baseline searched, one double at a time, for 1000 s == k + 0.5 EXACTLY, once
    with k even and once with k odd, and the double below it; half to even sends k + 0.5 to k for even k and to k + 1 for odd k"""
    out = []
    lu, ru = np.array([[160.0, 120.0]], np.float32), np.array([[144.0, 120.0]], np.float32)
    g = lambda tx: float(parts(TIE_CAM, TIE_CAM, cfg(IDENTITY, (tx, 0.0, 0.0), 60.0), lu, ru)["s"][0]) * 1000.0
    want = {0: None, 1: None}
    for k in range(2000, 2200):
        if want[k % 2] is not None:
            continue
        a, b = _flip(lambda tx: g(tx) >= k + 0.5, 0.05, 0.08)
        if g(b) == k + 0.5 and g(a) < k + 0.5:
            want[k % 2] = (k, a, b)
    assert want[0] is not None and want[1] is not None, "no baseline gives 1000 s == k.5 exactly"
    for k, a, b in (want[0], want[1]):
        out.append((_case("tie_%s" % ("even", "odd")[k % 2], TIE_CAM, TIE_CAM, cfg(IDENTITY, (b, 0.0, 0.0), 60.0), lu, ru), k if k % 2 == 0 else k + 1))
        out.append((_case("tie_%s_below" % ("even", "odd")[k % 2], TIE_CAM, TIE_CAM, cfg(IDENTITY, (a, 0.0, 0.0), 60.0), lu, ru), k))
    return out


_CASES = None


def cases():
    """built once per process"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    g = np.random.default_rng(11)
    # a rectified rig of distorted pinholes: depths of 0.5 .. 8 m against max_depth 3, one status in five 0
    lu = _grid(70, 1)
    z = g.uniform(0.5, 8.0, len(lu))
    st = (np.arange(len(lu)) % 5 != 0).astype(np.uint8)
    out.append(_case("rect", PIN, PIN, cfg(RECT["R"], RECT["t"], 3.0), lu, plant_from_left(PIN, PIN, RECT, lu, z), st))
    # a rotated, vertically offset right eye; PINHOLE_FULL on the left, MEI on the right, and the other way round
    lu = _grid(65, 2)
    out.append(_case("tilt_full_mei", FULL, MEI, cfg(TILT["R"], TILT["t"], 10.0), lu, plant_from_left(FULL, MEI, TILT, lu, g.uniform(0.5, 8.0, len(lu)))))
    lu = _grid(64, 3)
    ru = plant_from_left(MEI, FULL, TILT, lu, g.uniform(0.5, 8.0, len(lu)))
    ru[::7, 1] += 12.0                                                                     # every seventh match 12 px off its epipolar line
    out.append(_case("tilt_mei_full", MEI, FULL, cfg(TILT["R"], TILT["t"], 10.0), lu, ru))
    # SCARAMUZZA on either eye
    lu = _grid(63, 4)
    out.append(_case("sca_left", SCA, PIN, cfg(RECT["R"], RECT["t"], 10.0), lu, plant_from_left(SCA, PIN, RECT, lu, g.uniform(0.5, 8.0, len(lu)))))
    ru = _grid(33, 5)                                                                      # planted from the right eye: the rig inverted
    inv = dict(R=tuple(np.asarray(TILT["R"], F8).reshape(3, 3).T.reshape(9)), t=tuple(-(np.asarray(TILT["R"], F8).reshape(3, 3).T @ np.asarray(TILT["t"], F8))))
    out.append(_case("sca_right", PIN, SCA, cfg(TILT["R"], TILT["t"], 10.0), plant_from_left(SCA, PIN, inv, ru, g.uniform(0.5, 8.0, len(ru))), ru))
    # rays that are no rays: P.z <= 0 through MEI (xi == 1, 350 px off the centre) and SCARAMUZZA (740 px off), NaN pixels in either eye
    nan = np.float32(np.nan)
    out.append(_case("lift_mei", MEI1, PIN_PLAIN, cfg(RECT["R"], RECT["t"], 10.0), [[510.0, 120.0], [160.0, 120.0], [200.0, 130.0]], [[150.0, 120.0], [150.0, 120.0], [190.0, 130.0]]))
    out.append(_case("lift_sca", PIN_PLAIN, SCA, cfg(RECT["R"], RECT["t"], 10.0), [[160.0, 120.0], [200.0, 130.0]], [[900.0, 120.0], [190.0, 130.0]]))
    out.append(_case("nan", PIN, FULL, cfg(RECT["R"], RECT["t"], 10.0), [[nan, 120.0], [200.0, 130.0], [200.0, nan], [200.0, 130.0]], [[150.0, 120.0], [nan, 130.0], [190.0, 130.0], [190.0, 130.0]]))
    # behind: a negative disparity (s < 0 and u < 0), and a right eye turned by 170 degrees about y, for which the centre rays meet at s > 0 with u < 0
    out.append(_case("behind_both", PIN_PLAIN, PIN_PLAIN, cfg(RECT["R"], RECT["t"], 10.0), [[200.0, 130.0], [100.0, 90.0]], [[210.0, 130.0], [120.0, 90.0]]))
    back = rot(0.0, np.deg2rad(170.0), 0.0)
    out.append(_case("behind_u", PIN_PLAIN, PIN_PLAIN, cfg(back, (0.1, 0.0, 0.0), 10.0), [[160.0, 120.0], [162.0, 121.0]], [[160.0, 120.0], [161.0, 120.0]]))
    # no parallax: the same pixel in both eyes of a rectified rig, and a disparity of a tenth of a pixel
    out.append(_case("parallax", PIN_PLAIN, PIN_PLAIN, cfg(RECT["R"], RECT["t"], 60.0), [[200.0, 130.0], [100.0, 90.0]], [[200.0, 130.0], [99.9, 90.0]]))
    # the gates' boundaries.  parallax and epipolar: the two neighbouring doubles of the gate between which the comparison flips, for one match
    lu, ru = np.array([[200.25, 130.5]], np.float32), np.array([[198.75, 130.5]], np.float32)
    fires = lambda p: bool(depth(PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, min_parallax=p), lu, ru, [1])[1][0] == WHY["parallax"])
    a, b = _flip(fires, 1e-4, 1e-1)
    out.append(_case("parallax_below", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, min_parallax=a), lu, ru))
    out.append(_case("parallax_above", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, min_parallax=b), lu, ru))
    lu, ru = np.array([[200.25, 130.5]], np.float32), np.array([[190.25, 132.5]], np.float32)
    fires = lambda e: bool(depth(PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, max_epipolar=e), lu, ru, [1])[1][0] == WHY["epipolar"])
    a, b = _flip(fires, 1e-4, 1e-1)
    out.append(_case("epipolar_below", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, max_epipolar=a), lu, ru))
    out.append(_case("epipolar_above", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, max_epipolar=b), lu, ru))
    out += [c for c, _ in tie_cases()]
    # min_depth and max_depth in counts: depths of 1999, 2000 and 2001 counts against a bound of exactly 2000
    lu = np.array([[200.25, 130.5], [120.5, 100.25], [170.0, 60.0]], np.float32)
    ru = plant_from_left(PIN_PLAIN, PIN_PLAIN, RECT, lu, [1.99925, 2.00025, 2.00125])
    out.append(_case("min_2000", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 60.0, min_depth=2.0), lu, ru))
    out.append(_case("max_2000", PIN_PLAIN, PIN_PLAIN, cfg(IDENTITY, RECT["t"], 2.0), lu, ru))
    # the last count: 65535 and 65536 against max_depth 65.535, through a camera whose centre lies at (2, 2) so that the float pixels resolve a millimetre at 65 m
    far = camera("PINHOLE", (400.0, 400.0, 2.0, 2.0))
    wide = dict(R=IDENTITY, t=(0.5, 0.0, 0.0))
    lu = np.array([[2.0, 2.0], [2.0, 2.0]], np.float32)
    out.append(_case("last_count", far, far, cfg(IDENTITY, wide["t"], 65.535), lu, plant_from_left(far, far, wide, lu, [65.53525, 65.53625])))
    # the wavefront's edges: sets of 0, 1, 63, 64, 65 and 130 matches (an empty set between full ones, a set behind a longer one)
    for i, n in enumerate((64, 0, 130, 1, 63, 65)):
        lu = _grid(n, 20 + i)
        out.append(_case("edge_%d" % n, PIN, FULL, cfg(TILT["R"], TILT["t"], 6.0), lu, plant_from_left(PIN, FULL, TILT, lu, g.uniform(0.5, 8.0, n)) if n else np.zeros((0, 2), np.float32),
                         (np.arange(n) % 9 != 4).astype(np.uint8)))
    _CASES = out
    return out


def kb_case():
    """KANNALA_BRANDT on both eyes: held to a count, and to the reason wherever the restatement is not within 1e-9 relative of a gate"""
    g = np.random.default_rng(31)
    lu = _grid(66, 30)
    return _case("kb", KB, KB, cfg(TILT["R"], TILT["t"], 6.0), lu, plant_from_left(KB, KB, TILT, lu, g.uniform(0.5, 8.0, len(lu))))


def near_a_gate(c, rel=1e-9):
    """per point: the restatement is within `rel` relative of a gate's boundary (so a lift that differs in the last bits may decide otherwise)"""
    p = parts(c["left"], c["right"], c["cfg"], c["lu"], c["ru"])
    k = c["cfg"]
    with np.errstate(all="ignore"):
        near = lambda x, y: np.abs(x - y) <= rel * np.maximum(np.abs(x), np.abs(y))
        par = (F8(k["min_parallax"]) ** 2 * p["aa"]) * p["dd"]
        epi = F8(k["max_epipolar"]) ** 2 * (p["qz"] * p["qz"])
        frac = np.abs(1000.0 * p["s"] - np.floor(1000.0 * p["s"]) - 0.5)
        return near(p["den"], par) | near(p["e2"], epi) | (np.abs(p["s"]) <= rel) | (np.abs(p["u"]) <= rel) | (np.abs(p["qz"]) <= rel) | (frac <= rel * 1000.0 * np.abs(p["s"]))
